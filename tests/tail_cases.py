"""Shapes, operands and float64 references of the eval forward's dense tail (csrc/dense.hip behind Network._dense_tail:
confidence softmax, confidence pooling, pooling finish, pose heads, correspondence attention in the network's calling form),
shared by tests/test_tail_cases.py (CPU: the references against the literal module lines, the exact sets, the thresholds) and
tests/test_gpu_eval_tail.py (the kernels).  Everything here is built on the CPU, once per case, and handed out unchanged."""
import copy
import functools
import importlib
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the switches the shapes below are named for.  csrc/dense.hip keeps them as literals of its launchers; source_thresholds()
#      reads them back from the source text so that a changed literal fails tests/test_tail_cases.py instead of emptying a case
SOFTMAX_WIDE_ABOVE = 4096          # dcl_conf_softmax: more logits per crop than this take k_conf_softmax<1024> (16 waves)
POOL_SMALL_MAX_CROPS = 8           # dcl_conf_pool: up to this many crops ...
POOL_SMALL_MAX_LOGITS = 256 * 8    # ... of up to this many logits each run as ONE launch (k_conf_pool_small)
POOL_CHANNEL_BLOCK = 256           # channels per workgroup of the weighted column sums


def source_thresholds():
    """(softmax_wide_above, pool_small_max_crops, pool_small_max_logits) as csrc/dense.hip's launchers spell them"""
    src = open(os.path.join(ROOT, "dcl-net_amd", "csrc", "dense.hip")).read()
    wide = re.search(r"if \(n1 \+ n2 > (\d+)\) hipLaunchKernelGGL\(k_conf_softmax<1024>", src)
    small = re.search(r"if \(b <= (\d+) && n1 \+ n2 <= (\d+) \* (\d+)\) \{[^\n]*\n\s*hipLaunchKernelGGL\(k_conf_pool_small<(\d+)>", src)
    assert wide and small, "csrc/dense.hip: the launchers of dcl_conf_softmax / dcl_conf_pool are no longer spelled as expected"
    assert small.group(3) == small.group(4)
    return int(wide.group(1)), int(small.group(1)), int(small.group(2)) * int(small.group(3))


def pool_slices(b, c):
    """ops.conf_pool's slice count (restated; the GPU tests compare it with what the wrapper hands back)"""
    return max(1, min(64, 2048 // max(1, b * ((c + POOL_CHANNEL_BLOCK - 1) // POOL_CHANNEL_BLOCK))))


def slice_ranges(n, nslices):
    """[j0, j1) of every slice of a direction of n points (k_weighted_colsum); j0 >= j1: the slice owns no point"""
    per = (n + nslices - 1) // nslices
    return [(s * per, min(n, s * per + per)) for s in range(nslices)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def bound(ref64, module):
    """the project's rule (conf_pool_cases.compare): max(2 err_module, 1e-6 max|ref64|); returns (bound, err_module, max|ref64|)"""
    em = float((module.double() - ref64).abs().max())
    mx = float(ref64.abs().max())
    return max(2 * em, 1e-6 * mx), em, mx


def check(tag, name, got, ref64, module):
    """one output under the rule, with the one-line report"""
    lim, em, mx = bound(ref64, module)
    e = float((got.detach().cpu().double() - ref64).abs().max())
    print("tail\t%s\t%s\tmax|ref|=%.3g\terr=%.3g\terr_module=%.3g\tbound=%.3g" % (tag, name, mx, e, em, lim))
    assert e <= lim, (tag, name, e, em, mx)
    return e


# ------------------------------------------------------------------------------------------------ 1. softmax
# (b, n1, n2)
SOFTMAX_SHAPES = [
    (1, 1, 1),
    (3, 5, 7),
    (2, 1, 2047),
    (2, 2047, 1),
    (9, 1024, 1024),
    (2, 2048, 2048),              # L = 4096: the last size of the 256-thread form
    (2, 2048, 2049),              # L = 4097: the first of the 1024-thread form
    (1, 12288, 2048),             # the stress crop
    (2, 1025, 3100),              # L no multiple of 1024, n1 ends inside a wave
]
SOFTMAX_IDS = ["x".join(str(v) for v in s) for s in SOFTMAX_SHAPES]
LOGIT_SETS = ("gauss", "equal", "saturated", "opposed")


def logits(kind, b, n1, n2, seed):
    """(b, n1), (b, n2) fp32 logits.  gauss: N(0, 2^2); equal: one value everywhere; saturated: |x| up to 100 (the sigmoid
    saturates, expf(-x) overflows for the negative ones); opposed: crop 0 all -100 in direction 1 and all +100 in direction 2"""
    g = torch.Generator().manual_seed(seed)
    l1, l2 = torch.randn(b, n1, generator=g) * 2, torch.randn(b, n2, generator=g) * 2
    if kind == "equal":
        l1, l2 = torch.full((b, n1), 0.75), torch.full((b, n2), 0.75)
    elif kind == "saturated":
        l1, l2 = l1 * 25, l2 * 25
        l1.clamp_(-100, 100); l2.clamp_(-100, 100)
        l1.view(-1)[0], l2.view(-1)[-1] = -100.0, 100.0
    elif kind == "opposed":
        l1[0], l2[0] = -100.0, 100.0
    else:
        assert kind == "gauss"
    return l1.contiguous(), l2.contiguous()


def softmax64(l1, l2, wave_tree=16):
    """the definition in float64: conf = sigmoid(cat[l1, l2]), w = softmax(conf) per crop, wsum = w's two direction sums.
    wave_tree < 16 is the deliberately WRONG twin of a 1024-thread kernel that combines only the first `wave_tree` of its 16
    waves' sums (the 256-thread tree): elements j with (j % 1024) // 64 >= wave_tree are missing from the normaliser"""
    n1 = l1.shape[1]
    x = torch.cat([l1, l2], dim=1).double()
    conf = 1.0 / (1.0 + torch.exp(-x))
    e = torch.exp(conf - conf.max(dim=1, keepdim=True)[0])
    counted = ((torch.arange(x.shape[1]) % 1024) // 64 < wave_tree).double()
    w = e / (e * counted).sum(dim=1, keepdim=True)
    return dict(conf=conf, w=w, wsum=torch.stack([w[:, :n1].sum(1), w[:, n1:].sum(1)], dim=1))


def module_lines(l1, l2, F1=None, F2=None, affine=None):
    """the lines of the reference Network.forward (models/DCL_Net.py:217-228) in the dtype of the operands: logits (b, 1, n), F
    channel-major (b, c, n).  affine = (s1, t1, s2, t2): the fusers' trailing BatchNorms, applied to F1 / F2 BEFORE the pooling
    as the module does.  Returns conf (b, L), w (b, L), wsum (b, 2) and, with F, pooled (b, c)."""
    n1 = l1.shape[2]
    conf = torch.sigmoid(torch.cat([l1, l2], dim=2))
    conf_softmax = torch.softmax(conf, dim=2)
    out = dict(conf=conf.squeeze(1), w=conf_softmax.squeeze(1),
               wsum=torch.stack([conf_softmax[:, 0, :n1].sum(1), conf_softmax[:, 0, n1:].sum(1)], dim=1))
    if F1 is not None:
        if affine is not None:
            s1, t1, s2, t2 = affine
            F1 = F1 * s1[None, :, None] + t1[None, :, None]
            F2 = F2 * s2[None, :, None] + t2[None, :, None]
        F_p = torch.cat([F1, F2], dim=2)
        F_p_wei = torch.sum(F_p * conf_softmax, dim=2, keepdim=True)
        out["pooled"] = F_p_wei.squeeze(2)
    return out


@functools.lru_cache(maxsize=None)
def softmax_case(i, kind):
    """(l1, l2, float64 definition, fp32 module lines) of SOFTMAX_SHAPES[i] with the logit set `kind`"""
    b, n1, n2 = SOFTMAX_SHAPES[i]
    l1, l2 = logits(kind, b, n1, n2, 1000 + 10 * i + LOGIT_SETS.index(kind))
    return l1, l2, softmax64(l1, l2), module_lines(l1[:, None], l2[:, None])


# ------------------------------------------------------------------------------------------------ 2. pooling
# (b, n1, n2, c)
POOL_SHAPES = [
    (8, 1024, 1024, 1024),        # the last batch of the one-launch form
    (9, 1024, 1024, 1024),        # the first of the two-launch form
    (2, 1024, 1025, 1024),        # L = 2049 with few crops: two launches by the logit count
    (1, 1, 2047, 1024),           # direction 1 has fewer points than slices
    (1, 2047, 1, 1024),           # ... direction 2
    (3, 300, 170, 260),           # 260 = 256 + 4 channels: the channel count ends inside a 256-channel block
    (12, 100, 28, 1024),
]
POOL_IDS = ["x".join(str(v) for v in s) for s in POOL_SHAPES]
POOL_PAD, POOL_OFF = 24, 8        # F as a column block: pitch c + 24 floats, offset 8 floats


def pool64(l1, l2, F1, F2, affine=None, skip=None):
    """the definition in float64 on POINT-major F (b, n, c): w = softmax(sigmoid(logits)); P1 = sum_j w1_j F1_j, P2 likewise;
    finished = sA P1 + tA sum w1 + sB P2 + tB sum w2.  skip = (direction, j0, j1): the deliberately WRONG twin that leaves
    points j0..j1-1 of a direction out of its sum (a dropped slice)"""
    n1 = l1.shape[1]
    r = softmax64(l1, l2)
    w1, w2 = r["w"][:, :n1].clone(), r["w"][:, n1:].clone()
    if skip is not None:
        (w1, w2)[skip[0]][:, skip[1]:skip[2]] = 0.0
    P1 = torch.einsum("bjc,bj->bc", F1.double(), w1)
    P2 = torch.einsum("bjc,bj->bc", F2.double(), w2)
    r.update(P1=P1, P2=P2, pooled=P1 + P2)
    if affine is not None:
        sA, tA, sB, tB = (t.double() for t in affine)
        r["finished"] = sA * P1 + tA * r["wsum"][:, :1] + sB * P2 + tB * r["wsum"][:, 1:]
    return r


def pool_module(l1, l2, F1, F2, affine, dtype):
    """module_lines on the same operands in `dtype`: conf, wsum, pooled (no affine) and finished (with it)"""
    cm = lambda F: F.to(dtype).transpose(1, 2).contiguous()                                  # noqa: E731
    a, b2, F1c, F2c = l1[:, None].to(dtype), l2[:, None].to(dtype), cm(F1), cm(F2)
    m = module_lines(a, b2, F1c, F2c)
    m["finished"] = module_lines(a, b2, F1c, F2c, tuple(t.to(dtype) for t in affine))["pooled"]
    return m


def _pool_operands(b, n1, n2, c, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    return dict(l1=r(b, n1) * 2, l2=r(b, n2) * 2, F1=r(b, n1, c).relu_() * 1.5, F2=r(b, n2, c).relu_() * 1.5,
                affine=tuple(r(c) for _ in range(4)))


@functools.lru_cache(maxsize=None)
def pool_case(i):
    """operands of POOL_SHAPES[i] (logits N(0, 2^2), F = 1.5 relu(N(0, 1)) point-major, Gaussian affine vectors) with their
    float64 definition (`ref`) and the fp32 module lines (`module`)"""
    k = _pool_operands(*POOL_SHAPES[i], seed=2000 + i)
    k["ref"] = pool64(k["l1"], k["l2"], k["F1"], k["F2"], k["affine"])
    k["module"] = pool_module(k["l1"], k["l2"], k["F1"], k["F2"], k["affine"], torch.float32)
    return k


# exact sets: logits all 0, so conf = 0.5 and every weight is exp(0) / L = 1 / L with L a power of two; F small integers; the
# affine scales in {0.5, 1, 2}, the shifts integers: every sum of the definition is a dyadic rational fp32 holds, in any order
EXACT_POOL_SHAPES = [
    (3, 1000, 1048, 260),         # L = 2048, 3 crops: one launch
    (9, 1000, 1048, 260),         # ... 9 crops: two launches
    (2, 1000, 3096, 260),         # L = 4096: two launches by the logit count
]
EXACT_POOL_IDS = ["x".join(str(v) for v in s) for s in EXACT_POOL_SHAPES]


@functools.lru_cache(maxsize=None)
def exact_pool_case(i):
    b, n1, n2, c = EXACT_POOL_SHAPES[i]
    g = torch.Generator().manual_seed(2100 + i)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()                # noqa: E731
    k = dict(l1=torch.zeros(b, n1), l2=torch.zeros(b, n2), F1=ri(-4, 4, b, n1, c), F2=ri(-4, 4, b, n2, c),
             affine=(torch.pow(2.0, ri(-1, 1, c)), ri(-3, 3, c), torch.pow(2.0, ri(-1, 1, c)), ri(-3, 3, c)))
    k["ref"] = pool64(k["l1"], k["l2"], k["F1"], k["F2"], k["affine"])
    return k


# ------------------------------------------------------------------------------------------------ 3. finish
FINISH_COUNTS = [(1, 1), (2, 3), (5, 4), (8, 8), (96, 16), (7, 1)]       # (ns1, ns2): partials per crop and direction
FINISH_CHANNELS = (1024, 260)
FINISH_CROPS = (1, 9)
PARTS_SLICES = (1, 3, 4, 64)      # slice counts of the pose_heads_parts comparison


def finish64(part1, part2, ws, affine, ns1, ns2, drop_rest=False, swap_ws=False):
    """pooled = sA P1 + tA w0 + sB P2 + tB w1, P = a crop's partials added up, in float64: part1 (b * ns1, c), part2 (b * ns2, c).
    Deliberately WRONG twins: drop_rest leaves out the ns % 4 partials behind the last whole group of four; swap_ws swaps the
    two weight sums"""
    b, c = ws.shape[0], part1.shape[1]
    p1, p2 = part1.double().view(b, ns1, c), part2.double().view(b, ns2, c)
    if drop_rest:
        p1, p2 = p1[:, :ns1 // 4 * 4], p2[:, :ns2 // 4 * 4]
    w = ws.double()
    w0, w1 = (w[:, 1:], w[:, :1]) if swap_ws else (w[:, :1], w[:, 1:])
    sA, tA, sB, tB = (t.double() for t in affine)
    return sA * p1.sum(1) + tA * w0 + sB * p2.sum(1) + tB * w1


def finish_module(part1, part2, ws, affine, ns1, ns2):
    """the same composition in fp32 torch"""
    b, c = ws.shape[0], part1.shape[1]
    sA, tA, sB, tB = affine
    return ((sA * part1.view(b, ns1, c).sum(1) + tA * ws[:, :1]) + sB * part2.view(b, ns2, c).sum(1)) + tB * ws[:, 1:]


@functools.lru_cache(maxsize=None)
def finish_case(b, c, ns1, ns2, kind):
    """gauss: Gaussian partials, scales, shifts, weight sums in (0, 1).  exact: integer partials, scales in {0.5, 1, 2}, integer
    shifts, weight sums powers of two -- every sum exact in fp32"""
    g = torch.Generator().manual_seed(3000 + 1000 * b + c + 17 * ns1 + ns2)
    if kind == "gauss":
        r = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
        k = dict(part1=r(b * ns1, c), part2=r(b * ns2, c), ws=torch.rand(b, 2, generator=g), affine=tuple(r(c) for _ in range(4)))
    else:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()            # noqa: E731
        k = dict(part1=ri(-9, 9, b * ns1, c), part2=ri(-9, 9, b * ns2, c), ws=torch.pow(2.0, ri(-3, -1, b, 2)),
                 affine=(torch.pow(2.0, ri(-1, 1, c)), ri(-3, 3, c), torch.pow(2.0, ri(-1, 1, c)), ri(-3, 3, c)))
    k["ref"] = finish64(k["part1"], k["part2"], k["ws"], k["affine"], ns1, ns2)
    k["module"] = finish_module(k["part1"], k["part2"], k["ws"], k["affine"], ns1, ns2)
    return k


# ------------------------------------------------------------------------------------------------ 4. routes
# (b, n1, n2, crops checked against float64)
ROUTE_SHAPES = [
    (2, 128, 128, (0, 1)),
    (9, 128, 256, (0, 4, 8)),
    (9, 384, 128, (0, 4, 8)),
    (3, 12288, 2048, (0, 2)),     # the stress shape: routes a and c only
]
ROUTE_IDS = ["x".join(str(v) for v in s[:3]) for s in ROUTE_SHAPES]
HEADS_SEED = 9


def _package():
    return importlib.import_module("dcl-net_amd")


def heads_network():
    """a fresh CPU Network carrying the synth weights whose pose heads the route tests use"""
    dcl = _package()
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(64, 64), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, HEADS_SEED))
    return net.eval()


@functools.lru_cache(maxsize=None)
def _heads_double():
    net = heads_network()
    return copy.deepcopy(net.regressor_rot).double(), copy.deepcopy(net.regressor_trans).double()


def heads64(pooled):
    """the registered regressor_rot / regressor_trans modules (Head_MultiLayerPerceptron 1024 -> 512 -> 128 -> 9 | 3) in float64"""
    rot, trans = _heads_double()
    with torch.no_grad():
        x = pooled.double().unsqueeze(2)
        return rot(x).squeeze(2), trans(x).squeeze(2)


@functools.lru_cache(maxsize=None)
def route_case(i):
    """hidden activations H1 (b n1, 512), H2 (b n2, 512) (relu of Gaussians), the last fuser layer (512, 1024) + bias of either
    direction, logits, the four affine vectors; `ref`: per checked crop the float64 definition -- w = softmax(sigmoid(logits)),
    F = relu(H Wt + b), pooled = sA sum w1 F1 + tA sum w1 + sB sum w2 F2 + tB sum w2, then the two heads -- and `module`: the
    module lines in fp32 torch on the same operands"""
    b, n1, n2, crops = ROUTE_SHAPES[i]
    g = torch.Generator().manual_seed(4000 + i)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    k = dict(H1=r(b * n1, 512).relu_(), H2=r(b * n2, 512).relu_(), W1=r(512, 1024) * 0.05, b1=r(1024) * 0.1,
             W2=r(512, 1024) * 0.05, b2=r(1024) * 0.1, l1=r(b, n1) * 2, l2=r(b, n2) * 2, affine=tuple(r(1024) for _ in range(4)))
    sel = torch.tensor(crops)
    H1, H2 = k["H1"].view(b, n1, 512)[sel], k["H2"].view(b, n2, 512)[sel]
    l1, l2 = k["l1"][sel], k["l2"][sel]
    F = lambda H, W, bias, dt: torch.relu(H.to(dt) @ W.to(dt) + bias.to(dt))                 # noqa: E731
    ref = pool64(l1, l2, F(H1, k["W1"], k["b1"], torch.float64), F(H2, k["W2"], k["b2"], torch.float64), k["affine"])
    ref["o9"], ref["t3"] = heads64(ref["finished"])
    k["ref"] = ref
    k["module"] = pool_module(l1, l2, F(H1, k["W1"], k["b1"], torch.float32), F(H2, k["W2"], k["b2"], torch.float32), k["affine"],
                              torch.float32)
    return k


# ------------------------------------------------------------------------------------------------ 6. attention
# the smallest entries of tests/test_gpu_attention_plan.py per product kernel, both axes made ragged inside the plan entry
ATTN_CASES = {
    #        b   nq   nk  concurrent planes  kernels                                                          combine
    "C2": (128, 200, 61, 1, True, ("k_cross_attn_dma<4>",), False),
    "C1": (2, 200, 250, 1, True, ("k_cross_attn_dma<4>",), True),
    "C7": (128, 500, 61, 1, False, ("k_cross_attn_dma<8>",), False),
    "C3": (128, 200, 61, 2, True, ("k_attn_split_v", "k_attn_split_k", "k_cross_attn_split"), False),
}
ATTN_PITCH, ATTN_OFF = 136, 8     # Q and K as column blocks: pitch 136 floats, offset 8 floats
ATTN_GUARD = 3                    # guard rows behind the outputs
ATTN_TOL = 2e-5                   # x max(1, max|want|): the bound of test_cross_attention_matches_fp64


def attn64(Q, K, V):
    """Aligner (models/Modules.py:166-169) in float64 on point-major operands of ONE crop: softmax over the keys of K Q^T, then
    the weighted mean of V's rows"""
    A = torch.softmax(K.double() @ Q.double().t(), dim=0)          # (nk, nq)
    return A.t() @ V.double()


def attn_crops(b):
    return sorted({0, b // 2, b - 1})


@functools.lru_cache(maxsize=None)
def attn_case(b, nq, nk, kind="gauss"):
    """Q (b nq, 64), K (b nk, 64) (V2 is K itself, as in the network), V1 (b nk, 256) and the float64 result [O1 | O2] of the
    first, a middle and the last crop.
      gauss: Gaussian operands;  onekey..: as gauss (nk says it);
      zeroq: Q = 0, K and V1 small integers -- every score is 0, every weight 1, the output the exact mean of the values;
      neg60: every real score about -60 (K = -60 q0 / |q0|^2 + noise against Q = q0 + noise)"""
    g = torch.Generator().manual_seed(6000 + 131 * b + 7 * nq + nk + len(kind))
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    if kind == "zeroq":
        Q = torch.zeros(b * nq, 64)
        K = torch.randint(-8, 9, (b * nk, 64), generator=g).float()
        V1 = torch.randint(-8, 9, (b * nk, 256), generator=g).float()
    elif kind == "neg60":
        q0 = r(b, 1, 64)
        Q = (q0 + 0.05 * r(b, nq, 64)).reshape(-1, 64)
        K = (-60.0 * q0 / (q0 * q0).sum(2, keepdim=True) + 0.02 * r(b, nk, 64)).reshape(-1, 64)
        V1 = r(b * nk, 256)
    else:
        assert kind == "gauss"
        Q, K, V1 = r(b * nq, 64), r(b * nk, 64) * 0.3, r(b * nk, 256)
    want = {}
    for i in attn_crops(b):
        ks = slice(i * nk, (i + 1) * nk)
        want[i] = attn64(Q[i * nq:(i + 1) * nq], K[ks], torch.cat([V1[ks], K[ks]], dim=1))
    return dict(Q=Q, K=K, V1=V1, want=want)
