"""Operands, CPU models and bounds for the split-bf16 kernels (csrc/linear_split.hip: k_linear_split<EPI>; csrc/dense.hip:
k_cross_attn_split): tests/test_split_model.py checks the models and the bounds on the CPU, tests/test_gpu_split_arithmetic.py
runs the kernels on exactly the same bits.  CPU only, no test functions.  Every builder is seeded and cached; a reference is
computed once and shared -- never modify a returned tensor in place.

The model of the arithmetic: an fp32 value is split into three bf16 pieces by round-to-nearest-even (h, m, l), a product is
the six piece products of weight >= 2^-16 in the kernel's order (PRODUCTS), and one MFMA is modelled as the EXACT sum of its 16
products followed by ONE fp32 rounding into the accumulator.  That last part is an assumption about the matrix pipe, which is
why the GPU tests assert bounds derived by counting roundings, or bounds relative to an fp32 FMA chain, and never the model's
own figures."""
import functools
import math
import zlib

import torch

U = 2.0 ** -24                                   # one unit: the relative rounding error of one fp32 operation
TINY = 2.0 ** -126                               # the smallest normal fp32 / bf16
# (piece of x, piece of w) of the six products in accumulation order, 0 = h, 1 = m, 2 = l (linear_split.hip: l.h, h.l, m.m, m.h,
# h.m, h.h); the attention uses the same order with (K piece, Q piece) and (V piece, P piece)
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


# ------------------------------------------------------------------------------------------- the split and the GEMM models
def rn_bf16(v):
    return v.to(torch.bfloat16).float()


def trunc_bf16(v):
    """the mutant split: chop instead of round"""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(v, rnd=rn_bf16):
    """fp32 tensor -> (h, m, l) fp32 tensors holding bf16 values: h = RN(v), m = RN(v - h), l = RN(v - h - m)"""
    h = rnd(v)
    r = v - h
    m = rnd(r)
    l = rnd(r - m)
    return h, m, l


def _mfma_chunks(acc, a, b, drop, kc=16):
    """acc (fp32) += the six piece products of a (M, K) and b (K, N), 16 k at a time: exact 16-term sum, one rounding"""
    for c in range(0, a[0].shape[1], kc):
        for t, (i, j) in enumerate(PRODUCTS):
            if t != drop:
                acc = (acc.double() + a[i][:, c:c + kc] @ b[j][c:c + kc]).float()
    return acc


def _epilogue(acc, bias, relu):
    if bias is not None:
        acc = acc + bias
    return torch.relu(acc) if relu else acc


def model_split_gemm(x, Wt, drop=None, bias=None, relu=False, rnd=rn_bf16):
    """the split-bf16 GEMM core as modelled above; drop = t omits product t of PRODUCTS, rnd = trunc_bf16 is the chopping mutant"""
    xs = [p.double() for p in split3(x, rnd)]
    ws = [p.double() for p in split3(Wt, rnd)]
    acc = _mfma_chunks(torch.zeros(x.shape[0], Wt.shape[1]), xs, ws, drop)
    return _epilogue(acc, bias, relu)


def model_fma_chain(x, Wt, bias=None, relu=False):
    """k-ordered fp32 FMA chain (what an fp32-input MFMA computes): float64 a * b + acc is exact up to one rounding, rounded to
    fp32 once per step"""
    xd, wd = x.double(), Wt.double()
    acc = torch.zeros(x.shape[0], Wt.shape[1])
    for k in range(x.shape[1]):
        acc = torch.addcmul(acc.double(), xd[:, k:k + 1], wd[k:k + 1]).float()
    return _epilogue(acc, bias, relu)


def magnitude(x, Wt, bias=None):
    """sum_k |x_k| |w_k| (+ |bias|) per output, float64"""
    a = x.double().abs() @ Wt.double().abs()
    return a if bias is None else a + bias.double().abs()


def reference(x, Wt, bias=None, relu=False):
    want = x.double() @ Wt.double()
    if bias is not None:
        want = want + bias.double()
    return torch.relu(want) if relu else want


def unit_map(got, x, Wt, bias=None, relu=False):
    """|got - float64| / (2^-24 (sum |x||w| + |bias|)) per output; 0 where both vanish, inf where only the magnitude does"""
    err = (got.double() - reference(x, Wt, bias, relu)).abs()
    mag = magnitude(x, Wt, bias) * U
    out = err / mag
    out[(mag == 0) & (err == 0)] = 0.0
    return out


def units(got, x, Wt, bias=None, relu=False):
    """max over outputs of unit_map; NaN if anything in got is not finite"""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(unit_map(got, x, Wt, bias, relu).max())


def _gen(*key):
    """a generator seeded by the case's name and sizes (the same bits in every process)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _binades(shape, lo, hi, g):
    """randn * 2^randint(lo, hi) per element, both ends included"""
    return torch.randn(*shape, generator=g) * torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).float())


# ------------------------------------------------------------------------------------------- 3a: sparse rows
SPARSE_SHAPES = ((512, 64, 260), (300, 16, 130))


@functools.lru_cache(maxsize=None)
def sparse_case(M, K, N):
    """(x, Wt, bias, s): row i of x has s[i] = 1 + i % 3 non-zeros, the first at k = i % K (the only one where s = 1), the others
    at random other positions; values, weights and bias are randn * 2^randint(-20, 20) per element"""
    g = _gen("sparse", M, K, N)
    rows = torch.arange(M)
    s = 1 + rows % 3
    key = torch.rand(M, K, generator=g)
    key[rows, rows % K] = 2.0
    pos = key.topk(3, dim=1).indices                       # column 0 = i % K
    mask = torch.zeros(M, K, dtype=torch.bool)
    for q in range(3):
        sel = s > q
        mask[rows[sel], pos[sel, q]] = True
    x = torch.where(mask, _binades((M, K), -20, 20, g), torch.zeros(()))
    Wt = _binades((K, N), -20, 20, g)
    # every fourth one-hot row and every eighth weight column keep sign and binade but take the significand 1.0000000 11111111
    # 11111111b: harmless under rounding (h rounds up, the rest is one bit), the worst case of a split that chops (m and l both
    # at their largest: the three dropped products then come to 7.8 units)
    sel = (s == 1) & ((rows // 3) % 4 == 0)
    x[sel] = _ones_tail(x[sel])
    Wt[:, 3::8] = _ones_tail(Wt[:, 3::8])
    assert bool(((x != 0).sum(1) == s).all())
    return x, Wt, _binades((N,), -20, 20, g), s


def _ones_tail(v):
    e = torch.frexp(v)[1]
    return torch.where(v == 0, v, torch.sign(v) * torch.ldexp(torch.tensor(1.0 + 2.0 ** -7 - 2.0 ** -23), e - 1))


def sparse_bound_split(s, with_bias):
    """units allowed per output of a row with s non-zeros (derivation: test_sparse_rows_* in tests/test_gpu_split_arithmetic.py)"""
    return 6 * s + 1 + (1 if with_bias else 0)


def sparse_bound_fp32(s, with_bias):
    return s + 1 + (1 if with_bias else 0)


# ------------------------------------------------------------------------------------------- 3b: dense adversarial rows
DENSE_SETS = ("gaussian", "element_scales", "cancelling", "same_sign_l")
DENSE_M = 517
DENSE_KN = tuple((K, N) for K in (256, 480, 512) for N in (96, 260))
SPLIT_OVER_CHAIN = 1.5                            # units(split kernel) <= this x units(fp32 FMA chain), every case
FP32_OVER_CHAIN = 1.05                            # units(fp32 core)    <= this x units(fp32 FMA chain)


def _graded(shape, g, scale=1.0):
    """positive values (1 + p 2^-15 + q 2^-23) scale with p in [64, 127], q in [1, 63]: h = scale, m = p 2^-15 scale,
    l = q 2^-23 scale > 0 -- every second and every third piece has the same sign"""
    p = torch.randint(64, 128, shape, generator=g).double()
    q = torch.randint(1, 64, shape, generator=g).double()
    return ((1.0 + p * 2.0 ** -15 + q * 2.0 ** -23) * scale).float()


@functools.lru_cache(maxsize=None)
def dense_case(name, K, N, M=DENSE_M):
    """(x, Wt, bias) of operand set `name`"""
    g = _gen("dense", name, K, N, M)
    if name == "gaussian":
        x, Wt = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.05
    elif name == "element_scales":
        x, Wt = _binades((M, K), -30, 30, g), torch.randn(K, N, generator=g) * 0.05
    elif name == "cancelling":
        x1, w1 = torch.randn(M, K // 2, generator=g), torch.randn(K // 2, N, generator=g) * 0.05
        x, Wt = torch.cat([x1, -x1], 1), torch.cat([w1, w1 * (1.0 + 2.0 ** -12)], 0)
    elif name == "same_sign_l":
        x, Wt = _graded((M, K), g), _graded((K, N), g, 2.0 ** -4)
    else:
        raise KeyError(name)
    return x.contiguous(), Wt.contiguous(), torch.randn(N, generator=g)


@functools.lru_cache(maxsize=None)
def chain_units(name, K, N, M=DENSE_M):
    """units of the CPU fp32 FMA chain on dense_case / range_case (no bias, no ReLU): the yardstick of 3b and 3c"""
    x, Wt = (range_case(name) if name in RANGE_SETS else dense_case(name, K, N, M))[:2]
    return units(model_fma_chain(x, Wt), x, Wt)


# ------------------------------------------------------------------------------------------- 3c: range and non-finite
RANGE_SETS = ("huge", "tiny")
RANGE_SHAPE = (300, 64, 130)
H_OVERFLOWS = 0x7F7F8000                         # bit pattern of the smallest fp32 whose bf16 rounding is inf (3.3962e38)


@functools.lru_cache(maxsize=None)
def range_case(name):
    """(x, Wt): 'huge' = |x| in [2^100, 2^127) with |w| in [2^-100, 2^-96) (products stay finite, every piece of w is a normal
    bf16 number); 'tiny' = |x| in [2^-126, 2^-110) (third pieces are bf16 subnormals) with weights of order one"""
    M, K, N = RANGE_SHAPE
    g = _gen("range", name)
    sign = lambda shape: torch.randint(0, 2, shape, generator=g).float() * 2 - 1          # noqa: E731
    mant = lambda shape: 1.0 + torch.rand(shape, generator=g)                             # noqa: E731
    e = lambda shape, lo, hi: torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).float())   # noqa: E731
    if name == "huge":
        x = sign((M, K)) * mant((M, K)) * e((M, K), 100, 126)
        Wt = sign((K, N)) * mant((K, N)) * e((K, N), -100, -97)
    elif name == "tiny":
        x = sign((M, K)) * mant((M, K)) * e((M, K), -126, -111)
        Wt = _binades((K, N), -3, 3, g)
    else:
        raise KeyError(name)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(Wt).all())
    return x.contiguous(), Wt.contiguous()


def tiny_allowance(Wt):
    """sum_k 2^-126 |w_k| per output column: one fp32 minimum normal per term, whatever a flushed or inexact subnormal piece costs"""
    return TINY * Wt.double().abs().sum(0)


POISON_ROWS = (64, 100, 127, 516)                 # first / middle / last row of a 64-row wave block; the ragged last tile (M = 517)
POISON_COLS = (5, 129, 259)                       # first column tile, second column tile, the last column of the ragged one (N = 260)


# ------------------------------------------------------------------------------------------- 3d: the epilogues
POOL_FMAS = 66        # longest chain of the pooling epilogue: 64 FMAs in a lane, one shuffle add, one add across the two waves
ROWDOT_FMAS = 10      # 4 FMAs in a lane, 5 butterfly adds, the add of b3
POOL_CASES = ((1000, 64, 200, None), (1000, 480, 200, None), (1152, 64, 200, 384))       # (M, K, N, rows_per_crop)
POOL_W_STRIDE = 500                               # > rows_per_crop
ROWDOT_CASES = tuple((M, N) for N in (128, 96) for M in (1000, 37, 1, 0))
ROWDOT_K = 64


@functools.lru_cache(maxsize=None)
def pool_case(M, K, N, rows_per_crop):
    """(x, Wt, bias, roww): roww has zeros and negative entries; with rows_per_crop it is (crops, POOL_W_STRIDE), row j of x =
    (crop, point) weighing roww[crop, point]"""
    g = _gen("pool", M, K, N, rows_per_crop)
    x, Wt, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.1, torch.randn(N, generator=g)
    shape = (M,) if rows_per_crop is None else (M // rows_per_crop, POOL_W_STRIDE)
    roww = torch.randn(*shape, generator=g)
    roww[torch.rand(*shape, generator=g) < 0.2] = 0.0
    return x, Wt, bias, roww


def pool_row_weights(roww, M, rows_per_crop):
    return roww if rows_per_crop is None else roww[:, :rows_per_crop].reshape(M)


def pool_reference(x, Wt, bias, w, relu=True, tile=128):
    """float64 partials (ceil(M / 128), N) and their magnitudes sum_j |w_j| (sum_k |x||w| + |bias|)"""
    M, n = x.shape[0], Wt.shape[1]
    tiles = (M + tile - 1) // tile
    pad = lambda t: torch.cat([t, torch.zeros(tiles * tile - M, n, dtype=torch.float64)]).view(tiles, tile, n)   # noqa: E731
    wd = w.double().view(M, 1)
    return pad(wd * reference(x, Wt, bias, relu)).sum(1), pad(wd.abs() * magnitude(x, Wt, bias)).sum(1)


def model_pool(y, w, tile=128):
    """the pooling epilogue on fp32 activations y (M, N): an fp32 FMA chain over the rows of each 128-row tile"""
    M, n = y.shape
    tiles = (M + tile - 1) // tile
    yp = torch.cat([y, torch.zeros(tiles * tile - M, n)]).view(tiles, tile, n).double()
    wp = torch.cat([w, torch.zeros(tiles * tile - M)]).view(tiles, tile, 1).double()
    acc = torch.zeros(tiles, n)
    for j in range(tile):
        acc = torch.addcmul(acc.double(), yp[:, j], wp[:, j]).float()
    return acc


@functools.lru_cache(maxsize=None)
def rowdot_case(M, N):
    """(x, Wt, bias, w3 (N, 1) as a column of a padded buffer, b3)"""
    g = _gen("rowdot", M, N)
    x, Wt, bias = torch.randn(M, ROWDOT_K, generator=g), torch.randn(ROWDOT_K, N, generator=g) * 0.1, torch.randn(N, generator=g)
    return x, Wt, bias, torch.randn(N, 1, generator=g), torch.randn(1, generator=g)


def rowdot_reference(x, Wt, bias, w3, b3):
    """float64 out (M, 1) and magnitude sum_c |w3_c| (sum_k |x||w| + |bias_c|) + |b3|"""
    return (reference(x, Wt, bias, True) @ w3.double() + b3.double(),
            magnitude(x, Wt, bias) @ w3.double().abs() + b3.double().abs())


def model_rowdot(y, w3, b3):
    """the row-dot epilogue on fp32 hidden activations y (M, N): an fp32 FMA chain over the columns, then + b3"""
    acc = torch.zeros(y.shape[0], 1)
    for c in range(y.shape[1]):
        acc = torch.addcmul(acc.double(), y[:, c:c + 1].double(), w3[c:c + 1].double().view(1, 1)).float()
    return acc + b3


@functools.lru_cache(maxsize=None)
def pool_chain_units(M, K, N, rows_per_crop):
    x, Wt, bias, _ = pool_case(M, K, N, rows_per_crop)
    return units(model_fma_chain(x, Wt, bias), x, Wt, bias)


@functools.lru_cache(maxsize=None)
def rowdot_chain_units(M, N):
    x, Wt, bias, _, _ = rowdot_case(M, N)
    return units(model_fma_chain(x, Wt, bias), x, Wt, bias) if M else 0.0


def epilogue_bound(gemm_units, fmas):
    """units of sum |w_j| (sum |x||w| + |bias|) allowed to an epilogue output: every GEMM output it adds is off by at most
    gemm_units of its own magnitude (ReLU does not widen an error), and a summation tree whose longest chain has `fmas` operations
    is off by at most `fmas` units of the sum of its terms' magnitudes"""
    return gemm_units + fmas


# ------------------------------------------------------------------------------------------- 3e: dispatch
DISPATCH_N = 128
DISPATCH_BELOW, DISPATCH_FROM = 48896, 48897      # 191 and 192 row tiles of 256


# ------------------------------------------------------------------------------------------- 3f: attention
ATTN_B, ATTN_NQ, ATTN_NKS = 2, 300, (96, 1029)
ATTN_SPLITS = (0, 1, 4)                           # key split: 0 = what the launch plan picks on its own, 1 = forced whole, 4 = forced
ATTN_SETS = ("onehot", "cancel_v", "cancel_s", "v_spread", "gaussian")
ONEHOT_LEAD = 47.0                                # >= 40 + ln(1029): all other keys together weigh less than e^-40
ATTN_SPLIT_OVER_FP32 = 1.5


def onehot_keys(nk, nq=ATTN_NQ):
    """j*(i): every slot of the first two 32-key tiles, both sides of the tile boundaries where a 4-way key split cuts, the ragged
    last tile, then i % nk"""
    tiles = (nk + 31) // 32
    want = list(range(min(64, nk)))
    for z in range(1, 4):
        cut = 32 * (z * tiles // 4)
        want += [j for j in (cut - 2, cut - 1, cut, cut + 1) if 0 <= j < nk]
    want += list(range(32 * (tiles - 1), nk))
    want += [i % nk for i in range(nq)]
    return torch.tensor(want[:nq])


@functools.lru_cache(maxsize=None)
def attn_case(name, nk, b=ATTN_B, nq=ATTN_NQ):
    """(Q (b, nq, 64), K (b, nk, 64), V (b, nk, 320)) fp32; V[..., :256] is V1, V[..., 256:] is V2"""
    g = _gen("attn", name, nk, b, nq)
    V = torch.randn(b, nk, 320, generator=g)
    if name == "onehot":
        # key j = a sign code times magnitudes in [2, 2.5); query i = the key it selects: its logit is sum K^2 >= 256, every
        # other one a random walk of 64 steps of size ~5
        K = (torch.randint(0, 2, (b, nk, 64), generator=g).float() * 2 - 1) * (2.0 + 0.5 * torch.rand(b, nk, 64, generator=g))
        Q = K[:, onehot_keys(nk, nq)].clone()
        V = _binades((b, nk, 320), -20, 20, g)
    elif name == "cancel_v":
        # near-uniform weights over key pairs (v, -v (1 + 2^-12)); an odd last key holds zeros
        Q, K = torch.randn(b, nq, 64, generator=g) * 0.05, torch.randn(b, nk, 64, generator=g)
        V[:, 1::2] = -V[:, 0:nk - 1:2] * (1.0 + 2.0 ** -12)
        if nk % 2:
            V[:, nk - 1] = 0.0
    elif name == "cancel_s":
        # channel pairs (2c, 2c + 1): q equal, k opposite up to 2^-8: |q_c k_c| ~ 2^6 per channel, the logit of order one
        a = 8.0 * (1.0 + 0.25 * torch.rand(b, nq, 32, generator=g))
        k0 = 8.0 * (1.0 + 0.25 * torch.rand(b, nk, 32, generator=g)) * (torch.randint(0, 2, (b, nk, 32), generator=g).float() * 2 - 1)
        k1 = -k0 * (1.0 + 2.0 ** -8 * torch.randn(b, nk, 32, generator=g))
        Q = torch.stack([a, a], 3).reshape(b, nq, 64)
        K = torch.stack([k0, k1], 3).reshape(b, nk, 64)
    elif name == "v_spread":
        # key j's V row is scaled by 2^e_j, e_j in [-30, 30], and its logit is about -e_j ln(2) / 2: the large weights sit on
        # the small rows
        e = torch.randint(-30, 31, (b, nk, 1), generator=g).float()
        d = torch.randn(b, 1, 64, generator=g)
        d = d / d.norm(dim=2, keepdim=True)
        Q = 4.0 * d + 0.05 * torch.randn(b, nq, 64, generator=g)
        K = (-e * math.log(2.0) / 8.0) * d + 0.05 * torch.randn(b, nk, 64, generator=g)
        V = V * torch.exp2(e)
    elif name == "gaussian":
        Q, K = torch.randn(b, nq, 64, generator=g), torch.randn(b, nk, 64, generator=g)
    else:
        raise KeyError(name)
    return Q.contiguous(), K.contiguous(), V.contiguous()


@functools.lru_cache(maxsize=None)
def attn_reference(name, nk):
    """float64: (O (b, nq, 320), D = sum_j p_j |v_j| (b, nq, 320), S (b, nk, nq), sum_c |q_c||k_c| max)"""
    Q, K, V = attn_case(name, nk)
    S = torch.einsum("bjc,bic->bji", K.double(), Q.double())
    P = torch.softmax(S, dim=1)
    O = torch.einsum("bji,bjc->bic", P, V.double())
    D = torch.einsum("bji,bjc->bic", P, V.double().abs())
    qk = float(torch.einsum("bjc,bic->bji", K.double().abs(), Q.double().abs()).max())
    return O, D, S, qk


def units_attn(got, name, nk):
    """max over outputs of |got - float64| / (2^-24 sum_j p_j |v_j|), p from the float64 softmax; NaN if got is not finite"""
    O, D, _, _ = attn_reference(name, nk)
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - O).abs() / (D * U)).max())


def attn_apriori_units(nk):
    """what an fp32 form may be off by: one rounding per key in the P.V chain, and 64 for the weights (exp, the sum of the
    weights, the division, the rescales)"""
    return nk + 64


def effective_split(nk, split, b=ATTN_B, nq=ATTN_NQ):
    """the key split an 8-wave launch really gets (csrc/dense.hip: attn_key_split).  split = 0 leaves it to the launch plan
    (attn_auto_split8: a power of two up to 8 while it shortens the rounds of b ceil(nq / 256) workgroups over 256 CUs by 0.2
    of a workgroup time; b = 2, nq = 300: 4); a forced or picked split is granted at most one way per two 32-key tiles."""
    if split == 0:
        blocks, split = b * ((nq + 255) // 256), 1
        best = float((blocks + 255) // 256)
        for z in (2, 4, 8):
            cost = ((blocks * z + 255) // 256) / z
            if cost <= best - 0.2:
                best, split = cost, z
    return max(1, min(split, 8, ((nk + 31) // 32) // 2))


def onehot_c(nsplit):
    """roundings on the way from V[j*] to O[i] when one weight is exactly 1 (derivation: test_attention_one_hot_* in
    tests/test_gpu_split_arithmetic.py)"""
    return 10 if nsplit <= 1 else 12


def onehot_bound(V, jstar, nsplit):
    """(b, nq, 320) float64: c 2^-24 |V[j*]| + e^-40 max |V|"""
    b = V.shape[0]
    vs = torch.stack([V[i, jstar] for i in range(b)]).double()
    return onehot_c(nsplit) * U * vs.abs() + math.exp(-40.0) * float(V.abs().max())


def cancel_s_delta(qk_max):
    """what a logit may be off by: 4 k steps x 6 products + 1 roundings of a partial sum of at most sum |q||k|"""
    return 25 * U * qk_max


def model_split_attention(Q, K, V, drop_s=None, drop_pv=None, rnd=rn_bf16):
    """k_cross_attn_split as modelled above: S = K Q^T with six products per 16-channel step, p = exp(S - max) in fp32, split,
    six products per 16-key half tile into fp32 accumulators, fp32 sum of the weights, one division.  (The kernel's lazy maximum
    and its key split rescale by further factors; the model has the true maximum from the start.)"""
    b, nk = K.shape[0], K.shape[1]
    out = []
    for i in range(b):
        ks = [p.double() for p in split3(K[i], rnd)]
        qs = [p.double().t() for p in split3(Q[i], rnd)]
        S = _mfma_chunks(torch.zeros(nk, Q.shape[1]), ks, qs, drop_s)                     # (nk, nq)
        P = torch.exp(S - S.max(0, keepdim=True).values)
        lsum = torch.zeros(Q.shape[1])
        for j in range(nk):
            lsum = lsum + P[j]
        ps = [p.double().t() for p in split3(P, rnd)]                                      # (nq, nk)
        vs = [p.double() for p in split3(V[i], rnd)]
        O = torch.zeros(Q.shape[1], V.shape[2])
        for c in range(0, nk, 16):
            for t, (vi, pi) in enumerate(PRODUCTS):
                if t != drop_pv:
                    O = (O.double() + ps[pi][:, c:c + 16] @ vs[vi][c:c + 16]).float()
        out.append(O / lsum.view(-1, 1))
    return torch.stack(out)


def model_fp32_attention(Q, K, V):
    """the fp32 form: channel-ordered FMA chain for S, key-ordered FMA chain for P.V, fp32 exp, sum and division"""
    b, nk = K.shape[0], K.shape[1]
    out = []
    for i in range(b):
        S = model_fma_chain(K[i], Q[i].t().contiguous())
        P = torch.exp(S - S.max(0, keepdim=True).values)
        lsum = torch.zeros(Q.shape[1])
        for j in range(nk):
            lsum = lsum + P[j]
        out.append(model_fma_chain(P.t().contiguous(), V[i]) / lsum.view(-1, 1))
    return torch.stack(out)
