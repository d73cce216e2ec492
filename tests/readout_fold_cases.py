"""Operands, float64 twins, a CPU model and the bound for the folded read-out (csrc/linear_split.hip: EPI 4,
dcl_linear_split_gather_fwd; csrc/interp.hip: dcl_point_features_fold): tests/test_readout_fold_model.py checks the model on
the CPU, tests/test_gpu_readout_fold.py runs the kernels on the same bits.  CPU only, no test functions.  Every builder is
seeded and cached -- never modify a returned tensor in place.

The identity under test: with pf[:, col_m : col_m + c_m] = sum_i w[m, :, i] F_m[idx[m, :, i]] (the read-out's level m),

    pf @ W  =  pf[:, :K0] @ W[:K0]  +  sum over the folded levels m, i of  w[m, :, i] (F_m @ W[col_m : col_m + c_m])[idx[m, :, i]]

and the folded side is evaluated as  v = acc + bias;  v = fma(w[m, :, i], G_m[idx[m, :, i]], v)  for m ascending, i = 0, 1, 2."""
import functools
import zlib

import torch

import split_cases as SC

LEVEL_C = (32, 64, 128, 256)                     # channels of the four read-out levels (ops.BACKBONE_CHANNELS[2::2])
COL = (0, 32, 96, 224, 480)                      # their first columns in the read-out
K0 = {1: 224, 2: 96}                             # columns left to the GEMM with 1 / 2 levels folded


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _neighbours(M, R, g):
    """(M, 3) int32 rows in [0, R): many points share a row; rows 0 and R - 1 are named, R - 1 by the last point too"""
    idx = torch.randint(0, R, (M, 3), generator=g, dtype=torch.int32)
    idx[0, 0], idx[1, 2], idx[M - 1, 1] = R - 1, 0, R - 1
    return idx


def _weights(M, g):
    """(M, 3) float32: positive, sum 1 up to rounding -- what inverse-distance weights look like"""
    w = torch.rand(M, 3, generator=g) + 0.05
    return (w / w.sum(1, keepdim=True)).float()


# ------------------------------------------------------------------------------------------- the gather GEMM alone
GATHER_MN = tuple((M, N) for M in (256, 300, 768) for N in (128, 192))
GATHER_KFR = tuple((K, nfold, R) for K in (16, 224) for nfold in (1, 2) for R in (7, 300))
GATHER_C = {1: (64,), 2: (32, 64)}               # widths of the folded levels' feature tables in these cases


@functools.lru_cache(maxsize=None)
def gather_case(M, N, K, nfold, R):
    """x (M, K), W0 (K, N), bias (N,), F: nfold tables (R, c_l), Wl: nfold blocks (c_l, N), fw (nfold, M, 3), fi (nfold, M, 3)"""
    g = _gen("gather", M, N, K, nfold, R)
    x, W0, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.05, torch.randn(N, generator=g)
    F = tuple(torch.randn(R, c, generator=g) for c in GATHER_C[nfold])
    Wl = tuple(torch.randn(c, N, generator=g) * 0.05 for c in GATHER_C[nfold])
    fw = torch.stack([_weights(M, g) for _ in range(nfold)])
    fi = torch.stack([_neighbours(M, R, g) for _ in range(nfold)])
    return x, W0, bias, F, Wl, fw, fi


def gather_reference(x, W0, bias, F, Wl, fw, fi):
    """float64 twin: G in float64, interpolated in float64, then added -> (value before the activation, magnitude
    sum_k |x_k||w_k| + sum_{l,i} |fw| sum_k |F_k||W_k| + |bias|)"""
    want = x.double() @ W0.double() + (0.0 if bias is None else bias.double())
    mag = SC.magnitude(x, W0, bias)
    for l in range(len(F)):
        G, Gm = F[l].double() @ Wl[l].double(), F[l].double().abs() @ Wl[l].double().abs()
        for i in range(3):
            rows = fi[l, :, i].long()
            want = want + fw[l, :, i].double().view(-1, 1) * G[rows]
            mag = mag + fw[l, :, i].double().abs().view(-1, 1) * Gm[rows]
    return want, mag


def gather_units(got, want, mag, relu):
    """max over outputs of |got - float64| / (2^-24 magnitude); NaN if got is not finite"""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - (torch.relu(want) if relu else want)).abs() / (SC.U * mag)).max())


def gather_bound(K, widths, g_units=None):
    """Units of the magnitude T = A + sum_l B_l + |bias| an output may be off by (A = sum |x||w|, B_l = sum_i |fw| sum |F||W|):
      * the split product and the bias add: (6 s + 1) + 1 units of A + |bias| for a row of s = K non-zeros (tests/split_cases.py:
        sparse_bound_split; include/dclnet_hip.h);
      * a row of G_l comes out of a GEMM of c_l accumulations on the fp32-MFMA core, one rounding each of a partial sum of at most
        sum |F||W|: c_l units of its own magnitude (g_units[l] instead where another core computed it), and the weights of a
        point's three rows sum to that level's share B_l;
      * each of the 3 fused multiply-adds per folded level rounds the running value once, and the running value is at most T:
        3 units of T per level.
    A, the B_l and |bias| add up to T, so the first two lines together are at most max(6 K + 2, max c_l) units of T.  One more
    unit covers the second-order terms (every rounded quantity above is itself off by up to 2^-24 (6 K + 2) of its size: below
    2^-13 of a unit)."""
    g_units = list(widths) if g_units is None else list(g_units)
    return max([6 * K + 2] + g_units) + 3 * len(widths) + 1


# ------------------------------------------------------------------------------------------- the whole first layer, both routes
ROUTE_M, ROUTE_N, ROUTE_R = 768, 192, 300
ROUTE_OVER_TODAY = 1.5                           # max error of the folded route <= this x max error of today's route


@functools.lru_cache(maxsize=None)
def route_case():
    """Gaussian operands of the whole first layer: F (4 tables (R, c_m)), W (480, N), bias, w (4, M, 3), idx (4, M, 3)"""
    g = _gen("route")
    F = tuple(torch.randn(ROUTE_R, c, generator=g) for c in LEVEL_C)
    W = torch.randn(480, ROUTE_N, generator=g) * 0.05
    w = torch.stack([_weights(ROUTE_M, g) for _ in range(4)])
    idx = torch.stack([_neighbours(ROUTE_M, ROUTE_R, g) for _ in range(4)])
    return F, W, torch.randn(ROUTE_N, generator=g), w, idx


def unfolded_reference(F, W, bias, w, idx):
    """float64: the read-out (M, 480), then the layer"""
    pf = torch.cat([sum(w[m, :, i].double().view(-1, 1) * F[m].double()[idx[m, :, i].long()] for i in range(3)) for m in range(4)], 1)
    return pf @ W.double() + bias.double()


# ------------------------------------------------------------------------------------------- exact operands
EXACT_M, EXACT_N, EXACT_R = 300, 192, 37


@functools.lru_cache(maxsize=None)
def exact_case():
    """small integers in F, W and the bias, weights 0.5 / 0.25 / 0.25: every product and every sum of either route is exact in
    fp32 (read-out values are quarter integers of magnitude <= 4, a sum over 480 products stays below 2^13 quarters), so both
    routes give the bits of the float64 reference"""
    g = _gen("exact")
    F = tuple(torch.randint(-4, 5, (EXACT_R, c), generator=g).float() for c in LEVEL_C)
    W = torch.randint(-3, 4, (480, EXACT_N), generator=g).float()
    bias = torch.randint(-8, 9, (EXACT_N,), generator=g).float()
    w = torch.tensor([0.5, 0.25, 0.25]).repeat(4, EXACT_M, 1).contiguous()
    idx = torch.stack([_neighbours(EXACT_M, EXACT_R, g) for _ in range(4)])
    return F, W, bias, w, idx


def model_read_out(F, w, idx, levels=4):
    """the read-out's first `levels` levels in fp32, dcl_wsum3's order: fma(w2, f2, fma(w0, f0, w1 * f1))"""
    cols = []
    for m in range(levels):
        f = [F[m][idx[m, :, i].long()].double() for i in range(3)]
        ww = [w[m, :, i].double().view(-1, 1) for i in range(3)]
        t = (ww[1] * f[1]).float()
        t = (ww[0] * f[0] + t.double()).float()
        cols.append((ww[2] * f[2] + t.double()).float())
    return torch.cat(cols, 1)


def model_folded(F, W, bias, w, idx, nfold, drop_neighbour=None, drop_level=None, relu=False):
    """the folded route in fp32: the GEMM over the first 4 - nfold levels as an fp32 FMA chain (SC.model_fma_chain), G_m as one
    too, then one fma per (level, neighbour) in the kernel's order.  drop_neighbour = i / drop_level = m: the mutants that leave
    one neighbour of every folded level / one whole folded level out"""
    k0 = K0[nfold]
    v = SC.model_fma_chain(model_read_out(F, w, idx, 4 - nfold), W[:k0].contiguous()) + bias
    for m in range(4 - nfold, 4):
        if m == drop_level:
            continue
        G = SC.model_fma_chain(F[m], W[COL[m]:COL[m + 1]].contiguous())
        for i in range(3):
            if i != drop_neighbour:
                v = (w[m, :, i].double().view(-1, 1) * G[idx[m, :, i].long()].double() + v.double()).float()
    return torch.relu(v) if relu else v
